// nbldpc_amd/csrc/nbl_api_demod.cpp -- the demodulator in front of the decoder: nbl_set_demodulator*, the decodes from samples (with a
// prior, with gains), bit-LLR input, soft output and the iterative-demapping loop (nbl_demod.hip, nbl_soft.hip, nbl_idd.hip).
#include <cstdio>
#include "nbl_decoder.h"

// The per-symbol descriptor of the general demodulator (nbl_common.h, NblDemodPoint) from src [N p]; every index is checked here,
// before anything is indexed by it.
static nbl_status build_demod_desc(nbl_decoder *d, const nbl_demod_desc *dm, int m, std::vector<NblDemodPoint> &desc, std::vector<int> &tinv)
{
	const int N = d->g.N, p = d->g.p;
	const long long T = (long long)dm->n_mod_sym * m;
	std::vector<uint8_t> seen((size_t)T, 0);
	for (size_t i = 0; i < (size_t)N * p; i++) {
		const int t = dm->src[i];
		if (t < 0) continue;
		if (t >= T) { d->err = "demodulator source index out of range (label bit " + std::to_string(t) + " of code bit " + std::to_string(i) + ", L * m = " + std::to_string(T) + ")"; return NBL_ERR_ARG; }
		if (seen[t]) { d->err = "demodulator source: label bit " + std::to_string(t) + " is claimed twice"; return NBL_ERR_ARG; }
		seen[t] = 1;
	}
	tinv.assign((size_t)T, -1); // the inverse of src, for the prior-aware kernel: who claims label bit t
	for (size_t i = 0; i < (size_t)N * p; i++)
		if (dm->src[i] >= 0) tinv[dm->src[i]] = (int)i;
	NblDemodPoint none{};
	none.s = 0; none.nown = 0;
	for (int i = 0; i < 8; i++) none.own[i] = -1;
	desc.assign((size_t)N * (p + 1), none);
	for (int n = 0; n < N; n++) {
		NblDemodPoint *e = &desc[(size_t)n * (p + 1)];
		int pts[8], nt = 0;
		for (int j = 0; j < p; j++) {
			const int t = dm->src[(size_t)n * p + j];
			if (t < 0) continue;
			const int s = t / m;
			int k = 0;
			while (k < nt && pts[k] != s) k++;
			if (k == nt) pts[nt++] = s;
		}
		for (int x = 1; x < nt; x++) // ascending s
			for (int y = x; y > 0 && pts[y - 1] > pts[y]; y--) { const int tmp = pts[y]; pts[y] = pts[y - 1]; pts[y - 1] = tmp; }
		e[0].s = nt;
		for (int k = 0; k < nt; k++) e[1 + k].s = pts[k];
		for (int j = 0; j < p; j++) {
			const int t = dm->src[(size_t)n * p + j];
			if (t < 0) continue;
			int k = 0;
			while (pts[k] != t / m) k++;
			e[1 + k].own[t % m] = (int8_t)j;
			e[1 + k].nown++;
		}
	}
	return NBL_OK;
}

extern "C" nbl_status nbl_set_demodulator_ex(nbl_decoder *d, const nbl_demod_desc *dm, const nbl_demod_ext *ext)
{
	if (!d || !dm || !dm->src) return NBL_ERR_ARG;
	const int q = d->g.q, N = d->g.N, p = d->g.p;
	const int M = dm->mod_order;
	// every refusal comes before the device and the handle's state are touched: the demodulator set before stays usable
	if (M < 2 || M > 256 || (M & (M - 1))) {
		d->err = "nbl_set_demodulator: mod_order " + std::to_string(M) + " is not a power of two in 2 .. 256";
		return NBL_ERR_ARG;
	}
	const int metric = ext ? ext->metric : NBL_DEMOD_LOGSUM;
	if (metric != NBL_DEMOD_LOGSUM && metric != NBL_DEMOD_MAXLOG) {
		d->err = "nbl_set_demodulator_ex: unknown metric " + std::to_string(metric) + " (NBL_DEMOD_LOGSUM = 0, NBL_DEMOD_MAXLOG = 1)";
		return NBL_ERR_ARG;
	}
	const bool general = (M != 2 && M != q) || (ext && ext->force_general);
	if (dm->n_mod_sym <= 0) { d->err = "nbl_set_demodulator: n_mod_sym must be positive"; return NBL_ERR_ARG; }
	if ((general || M == q) && !dm->constellation) {
		d->err = "nbl_set_demodulator: this modulation order needs the constellation points (nbl_demod_desc.constellation)";
		return NBL_ERR_ARG;
	}
	const int m = ilog2(M);
	const size_t nsrc = (general || M == 2) ? (size_t)N * p : (size_t)N;
	std::vector<NblDemodPoint> desc;
	std::vector<int> tinv;
	if (general) {
		const nbl_status s = build_demod_desc(d, dm, m, desc, tinv);
		if (s) return s;
	} else {
		for (size_t i = 0; i < nsrc; i++)
			if (dm->src[i] >= dm->n_mod_sym) { d->err = "demodulator source index out of range"; return NBL_ERR_ARG; }
	}
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	d->tx = nbl_decoder::Tx(); // the transmitter's geometry repeats the demodulator's: set it again afterwards
	d->dm_order = 0;           // nothing is set until everything below has succeeded
	d->d_src.release();
	d->d_cons.release();
	d->d_dmdesc.release();
	d->d_tinv.release();
	nbl_status s;
	if (general) {
		if ((s = d->d_dmdesc.grow(d->err, desc.size() * sizeof(NblDemodPoint)))) return s;
		HIP_TRY(d, hipMemcpy(d->d_dmdesc, desc.data(), desc.size() * sizeof(NblDemodPoint), hipMemcpyHostToDevice));
		if ((s = d->d_tinv.grow(d->err, tinv.size() * sizeof(int)))) return s;
		HIP_TRY(d, hipMemcpy(d->d_tinv, tinv.data(), tinv.size() * sizeof(int), hipMemcpyHostToDevice));
	} else {
		if ((s = d->d_src.grow(d->err, nsrc * 4))) return s;
		HIP_TRY(d, hipMemcpy(d->d_src, dm->src, nsrc * 4, hipMemcpyHostToDevice));
	}
	d->h_cons.clear();
	if (dm->constellation) { // (BPSK: the demodulator does not need the points, the channel does)
		d->h_cons.assign(dm->constellation, dm->constellation + (size_t)2 * M);
		if ((s = d->d_cons.grow(d->err, (size_t)M * 16))) return s;
		HIP_TRY(d, hipMemcpy(d->d_cons, dm->constellation, (size_t)M * 16, hipMemcpyHostToDevice));
	}
	// the channel's buffers are sized per lane of dm_L symbols and the jump table is per symbol position: both are rebuilt for
	// the new L by the next channel call
	d->d_jump.release();
	d->d_jump_f.release();
	d->jump_f_pos = 0;
	d->noise_cap = 0;
	d->noise_pos = 0;
	d->dm_general = general;
	d->dm_metric = metric;
	d->dm_order = M;
	d->dm_L = dm->n_mod_sym;
	return NBL_OK;
}

extern "C" nbl_status nbl_set_demodulator(nbl_decoder *d, const nbl_demod_desc *dm) { return nbl_set_demodulator_ex(d, dm, nullptr); }

// received samples -> L_ch in the workspace: the BPSK / q-ary kernel, or the general one where nbl_set_demodulator_ex chose it
// d_prior [B][N p] (may be NULL): the prior-aware instance of the general kernel; the BPSK / q-ary kernels have no foreign position, a
// prior is inert there
// d_gain [B][L][2] (may be NULL): the gain-aware instances of either kernel
hipError_t launch_demod(nbl_decoder *d, const double *d_rx, double sigma, int B, const double *d_prior, const double *d_gain)
{
	if (d->dm_general)
		return nbl_launch_demod_general(d_rx, d->dm_L, sigma, d->dm_order, d->dm_metric, d->d_cons, d->d_dmdesc, d->g, d->w, B, d->stream, d_prior, d->d_tinv, d_gain);
	return nbl_launch_demod(d_rx, d->dm_L, sigma, d->dm_order, d->d_cons, d->d_src, d->g, d->w, B, d->stream, d_gain);
}

// host samples [B][L][2] -> d_rx (grown on demand), on the decoder's stream
static nbl_status stage_rx(nbl_decoder *d, const double *rx, int B)
{
	const size_t bytes = (size_t)B * d->dm_L * 16;
	if (nbl_status s = d->d_rx.grow(d->err, bytes)) return s;
	HIP_TRY(d, hipMemcpyAsync(d->d_rx, rx, bytes, hipMemcpyHostToDevice, d->stream));
	d->rx_gain = false;
	return NBL_OK;
}

// host gains [B][L][2] -> d_gain, on the decoder's stream
static nbl_status stage_gain(nbl_decoder *d, const double *gain, int B)
{
	const size_t bytes = (size_t)B * d->dm_L * 16;
	if (nbl_status s = d->d_gain.grow(d->err, bytes)) return s;
	HIP_TRY(d, hipMemcpyAsync(d->d_gain, gain, bytes, hipMemcpyHostToDevice, d->stream));
	d->rx_gain = true;
	return NBL_OK;
}

// nbl_decode_batch_samples, with a prior nbl_decode_batch_samples_prior, with gains nbl_decode_batch_samples_csi
static nbl_status decode_samples(nbl_decoder *d, const double *rx, const double *prior, double sigma, int32_t B, int32_t *out_sym,
                                 uint8_t *converged, int32_t *iters, const double *gain = nullptr)
{
	if (!d || !rx || !out_sym || B < 0 || !(sigma > 0)) return NBL_ERR_ARG;
	if (!d->dm_order) { d->err = "nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	if ((s = stage_rx(d, rx, B))) return s;
	if (gain && (s = stage_gain(d, gain, B))) return s;
	const double *d_gain = gain ? d->d_gain.p : nullptr;
	if (prior && d->dm_general) {
		const size_t pbytes = (size_t)B * d->g.N * d->g.p * 8;
		if ((s = d->d_prior.grow(d->err, pbytes))) return s;
		HIP_TRY(d, hipMemcpyAsync(d->d_prior, prior, pbytes, hipMemcpyHostToDevice, d->stream));
		HIP_TRY(d, launch_demod(d, d->d_rx, sigma, B, d->d_prior, d_gain));
	} else {
		HIP_TRY(d, launch_demod(d, d->d_rx, sigma, B, nullptr, d_gain));
	}
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	return read_back(d, d->w.out, d->w.done, d->w.iters, B, out_sym, converged, iters, hipMemcpyDeviceToHost, d->stream, true);
}

extern "C" nbl_status nbl_decode_batch_samples(nbl_decoder *d, const double *rx, double sigma, int32_t B, int32_t *out_sym,
                                               uint8_t *converged, int32_t *iters)
{
	return decode_samples(d, rx, nullptr, sigma, B, out_sym, converged, iters);
}

extern "C" nbl_status nbl_decode_batch_samples_prior(nbl_decoder *d, const double *rx, const double *prior, double sigma, int32_t B,
                                                     int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	return decode_samples(d, rx, prior, sigma, B, out_sym, converged, iters);
}

extern "C" nbl_status nbl_decode_batch_samples_csi(nbl_decoder *d, const double *rx, const double *gain, const double *prior, double sigma, int32_t B,
                                                   int32_t *out_sym, uint8_t *converged, int32_t *iters)
{
	return decode_samples(d, rx, prior, sigma, B, out_sym, converged, iters, gain);
}

// ---- bit-LLR input and batched soft output (nbl_soft.hip) ------------------------------------------------

extern "C" nbl_status nbl_decode_batch_bits_device(nbl_decoder *d, const double *d_bit_llr, int32_t B, int32_t *d_out_sym,
                                                   uint8_t *d_converged, int32_t *d_iters, void *stream)
{
	if (!d || !d_bit_llr || !d_out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	hipStream_t st = stream ? (hipStream_t)stream : d->stream;
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	HIP_TRY(d, nbl_launch_bits_to_lch(d_bit_llr, d->g, d->w, B, st));
	if ((s = run_iterations(d, nullptr, B, st))) return s; // (L_ch is in place: init_kernel leaves it alone)
	return read_back(d, d->w.out, d->w.done, d->w.iters, B, d_out_sym, d_converged, d_iters, hipMemcpyDeviceToDevice, st, false);
}

extern "C" nbl_status nbl_decode_batch_bits(nbl_decoder *d, const double *bit_llr, int32_t B, int32_t *out_sym, uint8_t *converged,
                                            int32_t *iters)
{
	if (!d || !bit_llr || !out_sym || B < 0) return NBL_ERR_ARG;
	if (B == 0) return NBL_OK;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	const size_t bytes = (size_t)B * d->g.N * d->g.p * 8;
	if ((s = d->d_lam.grow(d->err, bytes))) return s;
	HIP_TRY(d, hipMemcpyAsync(d->d_lam, bit_llr, bytes, hipMemcpyHostToDevice, d->stream));
	HIP_TRY(d, nbl_launch_bits_to_lch(d->d_lam, d->g, d->w, B, d->stream));
	if ((s = run_iterations(d, nullptr, B, d->stream))) return s;
	return read_back(d, d->w.out, d->w.done, d->w.iters, B, out_sym, converged, iters, hipMemcpyDeviceToHost, d->stream, true);
}

// what nbl_soft_output refuses, before the device is touched
static nbl_status soft_check(nbl_decoder *d, int32_t metric, uint32_t flags, const double *sym_llr, const double *bit_llr)
{
	if (!d) return NBL_ERR_ARG;
	if (d->prm.method == NBL_METHOD_OSD) { d->err = "nbl_soft_output: an OSD-only decoder (method 6) runs no iterations: there are no messages to form a posterior from"; return NBL_ERR_UNSUPPORTED; }
	if (!sym_llr && !bit_llr) { d->err = "nbl_soft_output: sym_llr and bit_llr are both NULL"; return NBL_ERR_ARG; }
	if (metric != NBL_SOFT_LOGSUM && metric != NBL_SOFT_MAXLOG) {
		d->err = "nbl_soft_output: unknown metric " + std::to_string(metric) + " (NBL_SOFT_LOGSUM = 0, NBL_SOFT_MAXLOG = 1)";
		return NBL_ERR_ARG;
	}
	if (flags & ~(uint32_t)NBL_SOFT_EXTRINSIC) {
		char hex[16];
		snprintf(hex, sizeof hex, "0x%x", (unsigned)(flags & ~(uint32_t)NBL_SOFT_EXTRINSIC));
		d->err = std::string("nbl_soft_output_ex: unknown flag bits ") + hex + " (NBL_SOFT_EXTRINSIC = 1)";
		return NBL_ERR_ARG;
	}
	if (d->last_B <= 0 || !d->w.Lch) { d->err = "nbl_soft_output: no decode call has run on this handle yet"; return NBL_ERR_ARG; }
	if (d->idd_sub) { d->err = std::string("nbl_soft_output") + NBL_IDD_SUB_TEXT; return NBL_ERR_ARG; }
	return NBL_OK;
}

// Where the c2v of the last decode call are: nbl_read_state's choice (below), handed to the kernel as a rule instead of being made per
// codeword on the host.  Every caller runs finish_pending first: the check-node pass of the last iteration may still be owed.
static NblSoftSrc soft_src(const nbl_decoder *d)
{
	NblSoftSrc s{};
	s.bufA = d->w.c2v;
	s.bufB = d->ws.c2v_alt;
	s.zeros = d->ws.c2v_zero;
	s.last = d->last_c2v ? d->last_c2v : d->w.c2v;
	s.last_shared = (d->ws.c2v_zero && s.last == d->ws.c2v_zero) ? 1 : 0;
	s.per_codeword = (d->last_fused && d->ws.c2v_alt && !d->prm.fixed_iters) ? 1 : 0;
	s.done = d->w.done;
	s.iters = d->w.iters;
	return s;
}

extern "C" nbl_status nbl_soft_output_device_ex(nbl_decoder *d, int32_t metric, uint32_t flags, double *d_sym_llr, double *d_bit_llr, void *stream)
{
	nbl_status s = soft_check(d, metric, flags, d_sym_llr, d_bit_llr);
	if (s) return s;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	hipStream_t st = stream ? (hipStream_t)stream : d->stream;
	if ((s = finish_pending(d, st))) return s;
	if ((s = widen_state(d, st))) return s;
	HIP_TRY(d, nbl_launch_soft_output(d->g, d->w.Lch, soft_src(d), d->last_B, metric, d_sym_llr, d_bit_llr, st, (flags & NBL_SOFT_EXTRINSIC) != 0));
	return NBL_OK;
}

extern "C" nbl_status nbl_soft_output_device(nbl_decoder *d, int32_t metric, double *d_sym_llr, double *d_bit_llr, void *stream)
{
	return nbl_soft_output_device_ex(d, metric, 0, d_sym_llr, d_bit_llr, stream);
}

extern "C" nbl_status nbl_soft_output_ex(nbl_decoder *d, int32_t metric, uint32_t flags, double *sym_llr, double *bit_llr)
{
	nbl_status s = soft_check(d, metric, flags, sym_llr, bit_llr);
	if (s) return s;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	const size_t B = (size_t)d->last_B, N = d->g.N;
	const size_t sym_bytes = B * N * (d->g.q - 1) * 8, bit_bytes = B * N * d->g.p * 8;
	if (sym_llr && (s = d->d_soft_sym.grow(d->err, sym_bytes))) return s;
	if (bit_llr && (s = d->d_soft_bit.grow(d->err, bit_bytes))) return s;
	if ((s = finish_pending(d))) return s;
	if ((s = widen_state(d))) return s;
	HIP_TRY(d, nbl_launch_soft_output(d->g, d->w.Lch, soft_src(d), d->last_B, metric, sym_llr ? d->d_soft_sym.p : nullptr,
	                                  bit_llr ? d->d_soft_bit.p : nullptr, d->stream, (flags & NBL_SOFT_EXTRINSIC) != 0));
	if (sym_llr) HIP_TRY(d, hipMemcpyAsync(sym_llr, d->d_soft_sym, sym_bytes, hipMemcpyDeviceToHost, d->stream));
	if (bit_llr) HIP_TRY(d, hipMemcpyAsync(bit_llr, d->d_soft_bit, bit_bytes, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_soft_output(nbl_decoder *d, int32_t metric, double *sym_llr, double *bit_llr)
{
	return nbl_soft_output_ex(d, metric, 0, sym_llr, bit_llr);
}

// ---- iterative demapping: the loop between the prior-aware demodulator and the decoder --------------------

// what the two _idd entry points refuse beyond what their plain forms refuse, before the device is touched
static nbl_status idd_check(nbl_decoder *d, const char *who, const nbl_idd_params *idd)
{
	const std::string w(who);
	if (!idd) { d->err = w + ": idd is NULL"; return NBL_ERR_ARG; }
	if (idd->passes < 1) { d->err = w + ": passes must be at least 1, got " + std::to_string(idd->passes); return NBL_ERR_ARG; }
	if (idd->soft_metric != NBL_SOFT_LOGSUM && idd->soft_metric != NBL_SOFT_MAXLOG) {
		d->err = w + ": unknown soft_metric " + std::to_string(idd->soft_metric) + " (NBL_SOFT_LOGSUM = 0, NBL_SOFT_MAXLOG = 1)";
		return NBL_ERR_ARG;
	}
	if (!d->dm_order) { d->err = w + ": nbl_set_demodulator has not been called"; return NBL_ERR_ARG; }
	if (idd->passes > 1 && d->prm.method == NBL_METHOD_OSD) {
		d->err = w + ": an OSD-only decoder (method 6) runs no iterations: there are no messages to form a prior from, passes must be 1";
		return NBL_ERR_UNSUPPORTED;
	}
	return NBL_OK;
}

// passes 1 .. idd->passes over the samples d_rx0 [B][L][2] (only ever read); leaves out / converged / iters / pass of every codeword at
// its batch position in d->idd.res_*.  One stream synchronisation per pass that has a successor: the survivor count sizes the next grids.
// d_gain0 [B][L][2] (may be NULL): the gains of those samples; the survivors' rows are gathered with their samples.
nbl_status run_idd(nbl_decoder *d, const double *d_rx0, double sigma, int B, const nbl_idd_params *idd, const double *d_gain0)
{
	nbl_decoder::Idd &x = d->idd;
	const int N = d->g.N, Np = d->g.N * d->g.p, rx_row = 2 * d->dm_L;
	nbl_status s;
	if ((s = x.res_out.grow(d->err, (size_t)B * N * 4))) return s;
	if ((s = x.res_iters.grow(d->err, (size_t)B * 4))) return s;
	if ((s = x.res_pass.grow(d->err, (size_t)B * 4))) return s;
	if ((s = x.res_done.grow(d->err, (size_t)B))) return s;
	const double *rx = d_rx0, *prior = nullptr, *gain = d_gain0;
	const int *idx = nullptr;
	int n = B, side = 0;
	for (int k = 1;; k++) {
		HIP_TRY(d, launch_demod(d, rx, sigma, n, prior, gain));
		if ((s = run_iterations(d, nullptr, n, d->stream))) return s;
		HIP_TRY(d, nbl_launch_idd_scatter(d->w.out, d->w.done, d->w.iters, idx, n, N, k, x.res_out, x.res_done, x.res_iters, x.res_pass, d->stream));
		if (k == idd->passes) break;
		int live = 0;
		HIP_TRY(d, nbl_launch_compact(d->w.done, n, d->ws.active, (int *)d->w.n_act, d->stream));
		HIP_TRY(d, hipMemcpyAsync(&live, d->w.n_act, sizeof live, hipMemcpyDeviceToHost, d->stream));
		HIP_TRY(d, hipStreamSynchronize(d->stream));
		if (live <= 0) break;
		if (live > n) { d->err = "iterative demapping: the active list is longer than the batch"; return NBL_ERR_HIP; }
		if ((s = x.ext.grow(d->err, (size_t)n * Np * 8))) return s;
		if ((s = x.prior.grow(d->err, (size_t)live * Np * 8))) return s;
		if ((s = x.rx[side].grow(d->err, (size_t)live * rx_row * 8))) return s;
		if ((s = x.idx[side].grow(d->err, (size_t)live * 4))) return s;
		if ((s = finish_pending(d))) return s; // (the survivors' extrinsic LLRs come from the c2v of the last iteration)
		if ((s = widen_state(d))) return s;    // (nbl_create_fht32: that c2v, widened, as nbl_soft_output would read it)
		HIP_TRY(d, nbl_launch_soft_output(d->g, d->w.Lch, soft_src(d), n, idd->soft_metric, nullptr, x.ext, d->stream, true));
		if (gain && (s = x.gain[side].grow(d->err, (size_t)live * rx_row * 8))) return s;
		HIP_TRY(d, nbl_launch_idd_gather(d->ws.active, live, rx, rx_row, x.ext, Np, idx, x.rx[side], x.prior, x.idx[side], d->stream, gain,
		                                 gain ? x.gain[side].p : nullptr));
		rx = x.rx[side];
		if (gain) gain = x.gain[side];
		idx = x.idx[side];
		prior = x.prior;
		side ^= 1;
		n = live;
	}
	d->idd_sub = true;
	return NBL_OK;
}

// a demodulator without a foreign position (BPSK / q-ary, not forced general): every pass is the same decode, so pass 1 is run alone
// and a codeword that did not converge is reported with the pass the definition ends on
static void idd_inert_passes(const nbl_idd_params *idd, const uint8_t *conv, int32_t B, int32_t *passes_used)
{
	if (passes_used)
		for (int b = 0; b < B; b++) passes_used[b] = conv[b] ? 1 : idd->passes;
}

// nbl_decode_batch_samples_idd, with gains nbl_decode_batch_samples_idd_csi
static nbl_status decode_samples_idd(nbl_decoder *d, const char *who, const double *rx, const double *gain, double sigma, int32_t B,
                                     const nbl_idd_params *idd, int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used)
{
	if (!d || !rx || !out_sym || B < 0 || !(sigma > 0)) return NBL_ERR_ARG;
	nbl_status s = idd_check(d, who, idd);
	if (s) return s;
	if (B == 0) return NBL_OK;
	if (idd->passes == 1 || !d->dm_general) {
		std::vector<uint8_t> conv(converged ? 0 : (size_t)B);
		uint8_t *cv = converged ? converged : conv.data();
		if ((s = decode_samples(d, rx, nullptr, sigma, B, out_sym, cv, iters, gain))) return s;
		idd_inert_passes(idd, cv, B, passes_used);
		return NBL_OK;
	}
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	if ((s = ensure_workspace(d, B))) return s;
	if ((s = stage_rx(d, rx, B))) return s;
	if (gain && (s = stage_gain(d, gain, B))) return s;
	if ((s = run_idd(d, d->d_rx, sigma, B, idd, gain ? d->d_gain.p : nullptr))) return s;
	if ((s = read_back(d, d->idd.res_out, d->idd.res_done, d->idd.res_iters, B, out_sym, converged, iters, hipMemcpyDeviceToHost, d->stream, false))) return s;
	if (passes_used) HIP_TRY(d, hipMemcpyAsync(passes_used, d->idd.res_pass, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	return NBL_OK;
}

extern "C" nbl_status nbl_decode_batch_samples_idd(nbl_decoder *d, const double *rx, double sigma, int32_t B, const nbl_idd_params *idd,
                                                   int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used)
{
	return decode_samples_idd(d, "nbl_decode_batch_samples_idd", rx, nullptr, sigma, B, idd, out_sym, converged, iters, passes_used);
}

extern "C" nbl_status nbl_decode_batch_samples_idd_csi(nbl_decoder *d, const double *rx, const double *gain, double sigma, int32_t B,
                                                       const nbl_idd_params *idd, int32_t *out_sym, uint8_t *converged, int32_t *iters,
                                                       int32_t *passes_used)
{
	return decode_samples_idd(d, gain ? "nbl_decode_batch_samples_idd_csi" : "nbl_decode_batch_samples_idd", rx, gain, sigma, B, idd, out_sym,
	                          converged, iters, passes_used);
}

extern "C" nbl_status nbl_decode_batch_resident_idd(nbl_decoder *d, int32_t slot, double sigma, int32_t B, const nbl_idd_params *idd,
                                                    int32_t *out_sym, uint8_t *converged, int32_t *iters, int32_t *passes_used)
{
	if (!d || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0)) return NBL_ERR_ARG;
	nbl_status s = idd_check(d, "nbl_decode_batch_resident_idd", idd);
	if (s) return s;
	if (idd->passes == 1 || !d->dm_general) {
		std::vector<uint8_t> conv(converged ? 0 : (size_t)B);
		uint8_t *cv = converged ? converged : conv.data();
		if ((s = nbl_decode_batch_resident(d, slot, sigma, B, out_sym, cv, iters))) return s;
		idd_inert_passes(idd, cv, B, passes_used);
		return NBL_OK;
	}
	if (nbl_status rs = resident_check(d, slot, B, out_sym)) return rs;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	if ((s = ensure_workspace(d, B))) return s;
	if (d->tx.on) d->tx.dec_B[slot] = 0;
	if ((s = run_idd(d, d->d_rxs[slot], sigma, B, idd, d->slot_gain[slot] ? d->d_gains[slot].p : nullptr))) return s; // (the slot's samples and gains are only read)
	if (out_sym) HIP_TRY(d, hipMemcpyAsync(out_sym, d->idd.res_out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToHost, d->stream));
	if (d->tx.on) { // the slot keeps the final words for nbl_count_errors
		if ((s = d->tx.dec[slot].grow(d->err, (size_t)B * d->g.N * 4))) return s;
		HIP_TRY(d, hipMemcpyAsync(d->tx.dec[slot], d->idd.res_out, (size_t)B * d->g.N * 4, hipMemcpyDeviceToDevice, d->stream));
	}
	if (converged) HIP_TRY(d, hipMemcpyAsync(converged, d->idd.res_done, (size_t)B, hipMemcpyDeviceToHost, d->stream));
	if (iters) HIP_TRY(d, hipMemcpyAsync(iters, d->idd.res_iters, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	if (passes_used) HIP_TRY(d, hipMemcpyAsync(passes_used, d->idd.res_pass, (size_t)B * 4, hipMemcpyDeviceToHost, d->stream));
	HIP_TRY(d, hipStreamSynchronize(d->stream));
	if (d->tx.on) d->tx.dec_B[slot] = B;
	return NBL_OK;
}

// Diagnostic only (not part of include/nbldpc.h): device time in milliseconds of ONE launch of the demodulator on the samples a slot
// holds, between two events on the decoder's stream -- with_prior != 0: the prior-aware instance, on an all-zero prior (the kernel's
// work does not depend on the values).  For tools/idd_pass.py.
// with_gain != 0 (nbl_debug_time_demod_csi): the gain-aware instance, on the slot's own gains where it holds some, else on all-zero
// gains (the kernel's work does not depend on the values).  For tools/fading_fer.py.
static nbl_status time_demod(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t with_prior, int32_t with_gain, double *ms)
{
	if (!d || !ms || B <= 0 || slot < 0 || slot > 1 || !(sigma > 0) || !d->dm_order || d->rxs_B[slot] != B) return NBL_ERR_ARG;
	d->err.clear();
	HIP_TRY(d, hipSetDevice(d->device));
	nbl_status s = ensure_workspace(d, B);
	if (s) return s;
	const double *prior = nullptr;
	if (with_prior && d->dm_general) {
		const size_t pbytes = (size_t)B * d->g.N * d->g.p * 8;
		if ((s = d->d_prior.grow(d->err, pbytes))) return s;
		HIP_TRY(d, hipMemsetAsync(d->d_prior, 0, pbytes, d->stream));
		prior = d->d_prior;
	}
	const double *gain = nullptr;
	if (with_gain && d->slot_gain[slot]) gain = d->d_gains[slot];
	else if (with_gain) {
		const size_t gbytes = (size_t)B * d->dm_L * 16;
		if ((s = d->d_gain.grow(d->err, gbytes))) return s;
		HIP_TRY(d, hipMemsetAsync(d->d_gain, 0, gbytes, d->stream));
		d->rx_gain = false;
		gain = d->d_gain;
	}
	hipEvent_t a = nullptr, b = nullptr;
	HIP_TRY(d, hipEventCreate(&a));
	HIP_TRY(d, hipEventCreate(&b));
	hipError_t e = hipEventRecord(a, d->stream);
	if (e == hipSuccess) e = launch_demod(d, d->d_rxs[slot], sigma, B, prior, gain);
	if (e == hipSuccess) e = hipEventRecord(b, d->stream);
	if (e == hipSuccess) e = hipEventSynchronize(b);
	float t = 0;
	if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
	(void)hipEventDestroy(a);
	(void)hipEventDestroy(b);
	HIP_TRY(d, e);
	*ms = t;
	return NBL_OK;
}

extern "C" nbl_status nbl_debug_time_demod(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t with_prior, double *ms)
{
	return time_demod(d, slot, sigma, B, with_prior, 0, ms);
}

extern "C" nbl_status nbl_debug_time_demod_csi(nbl_decoder *d, int32_t slot, double sigma, int32_t B, int32_t with_prior, int32_t with_gain, double *ms)
{
	return time_demod(d, slot, sigma, B, with_prior, with_gain, ms);
}
