// nbldpc_amd/host/capi.cpp -- small C entry points over the host layer for the Python tests (ctypes).
#include <cstdlib>
#include <cstring>
#include <thread>
#include "link.h"

extern "C" {

// Run the link chain of every lane for `frames` cycles WITHOUT decoding and return what the reference's chain produced:
// L_ch [frames*P][N][q-1] (frame-major, b = f*P + lane), tx_code [frames*P][N], tx_msg [frames*P][K].  No GPU needed.
int nblh_frontend(const char *profile, double ebn0, int frames, double *L_ch, int *tx_code, int *tx_msg, double *sigma_out)
{
	CSimulation sim;
	if (sim.Initial(profile) != 0) return -1;
	sim.EbN0 = ebn0;
	// host-only CNBLDPC use: parse + encoder, no device (Initial would need a GPU) -> replicate the needed part
	CLink link;
	link.sim = sim;
	CNBLDPC &code = link.code;
	// the front-end needs the graph and the encoder only: no device decoder is created (device = -1)
	if (!code.Initial(link.sim, -1)) return -2;
	const int P = sim.parallel, N = code.CodeLen, K = code.CodeLen - code.ChkLen, w = code.GFq - 1;
	std::vector<std::unique_ptr<CComm>> lanes;
	for (int i = 0; i < P; i++) {
		lanes.emplace_back(new CComm());
		if (!lanes.back()->Initial(link.sim, i, &code)) return -3;
		lanes.back()->SetEbN0(link.sim, i);
	}
	if (sigma_out) *sigma_out = lanes[0]->sigma_n;
	// lanes are independent (own RNG, PN register, buffers): run them on host threads, frame after frame per lane
	auto work = [&](int lo, int hi) {
		for (int i = lo; i < hi; i++) {
			CComm &c = *lanes[i];
			for (int f = 0; f < frames; f++) {
				c.FrontEnd();
				const size_t b = (size_t)f * P + i;
				memcpy(L_ch + b * N * w, c.RX_LLR_SYM.data(), sizeof(double) * N * w);
				if (tx_code) for (int n = 0; n < N; n++) tx_code[b * N + n] = c.TX_CODE_SYM[n];
				if (tx_msg) for (int n = 0; n < K; n++) tx_msg[b * K + n] = c.TX_MSG_SYM[n];
			}
		}
	};
	int T = (int)std::thread::hardware_concurrency();
	if (const char *e = getenv("NBL_HOST_THREADS")) T = atoi(e);
	if (T > 16) T = 16;
	if (T > P) T = P;
	if (T <= 1) work(0, P);
	else {
		std::vector<std::thread> th;
		for (int t = 0; t < T; t++) th.emplace_back(work, (int)((long long)P * t / T), (int)((long long)P * (t + 1) / T));
		for (auto &x : th) x.join();
	}
	return 0;
}

// Host link chain up to and including Channel_AWGN for `frames` cycles (no GPU): received samples rx [frames*P][L][2], the
// constellation index of every transmitted symbol tx_index [frames*P][L] and each lane's generator state in front of each
// frame state [frames*P][3] -- what the device-side channel is given, and what it must reproduce.
int nblh_channel(const char *profile, double ebn0, int frames, double *rx, unsigned char *tx_index, unsigned int *state, double *sigma_out)
{
	CSimulation sim;
	if (sim.Initial(profile) != 0) return -1;
	sim.EbN0 = ebn0;
	CLink link;
	link.sim = sim;
	CNBLDPC &code = link.code;
	if (!code.Initial(link.sim, -1)) return -2;
	const int P = sim.parallel;
	std::vector<std::unique_ptr<CComm>> lanes;
	for (int i = 0; i < P; i++) {
		lanes.emplace_back(new CComm());
		if (!lanes.back()->Initial(link.sim, i, &code)) return -3;
		lanes.back()->SetEbN0(link.sim, i);
	}
	if (sigma_out) *sigma_out = lanes[0]->sigma_n;
	const int L = lanes[0]->MOD_SYM_LEN;
	auto work = [&](int lo, int hi) {
		for (int i = lo; i < hi; i++) {
			CComm &c = *lanes[i];
			for (int f = 0; f < frames; f++) {
				const size_t b = (size_t)f * P + i;
				state[b * 3 + 0] = (unsigned int)(c.Rand.IX % 61967ul);
				state[b * 3 + 1] = (unsigned int)(c.Rand.IY % 63443ul);
				state[b * 3 + 2] = (unsigned int)(c.Rand.IZ % 63599ul);
				c.FrontEndToChannel();
				for (int s = 0; s < L; s++) {
					rx[(b * L + s) * 2] = c.RX_MOD_SYM[s].Real;
					rx[(b * L + s) * 2 + 1] = c.RX_MOD_SYM[s].Image;
					tx_index[b * L + s] = c.TX_MOD_IDX[s];
				}
			}
		}
	};
	int T = (int)std::thread::hardware_concurrency();
	if (const char *e = getenv("NBL_HOST_THREADS")) T = atoi(e);
	if (T > 16) T = 16;
	if (T > P) T = P;
	if (T <= 1) work(0, P);
	else {
		std::vector<std::thread> th;
		for (int t = 0; t < T; t++) th.emplace_back(work, (int)((long long)P * t / T), (int)((long long)P * (t + 1) / T));
		for (auto &x : th) x.join();
	}
	return L;
}

// nblh_channel over the Rayleigh block-fading channel (CComm::Channel_Rayleigh, `coherence` samples per gain), whatever NBL_CHANNEL
// says: additionally the per-sample gains gain [frames*P][L][2]; *draws_out = the uniform draws one frame moves a lane's generator.
int nblh_channel_fading(const char *profile, double ebn0, int frames, int coherence, double *rx, double *gain, unsigned char *tx_index,
                        unsigned int *state, double *sigma_out, unsigned long long *draws_out)
{
	if (coherence < 1) return -4;
	CSimulation sim;
	if (sim.Initial(profile) != 0) return -1;
	sim.EbN0 = ebn0;
	CLink link;
	link.sim = sim;
	CNBLDPC &code = link.code;
	if (!code.Initial(link.sim, -1)) return -2;
	const int P = sim.parallel;
	std::vector<std::unique_ptr<CComm>> lanes;
	for (int i = 0; i < P; i++) {
		lanes.emplace_back(new CComm());
		if (!lanes.back()->Initial(link.sim, i, &code)) return -3;
		lanes.back()->fade_model = NBL_FADING_RAYLEIGH;
		lanes.back()->fade_block = coherence;
		lanes.back()->GAIN.assign(lanes.back()->MOD_SYM_LEN, CComplex());
		lanes.back()->SetEbN0(link.sim, i);
	}
	if (sigma_out) *sigma_out = lanes[0]->sigma_n;
	if (draws_out) *draws_out = lanes[0]->ChannelDraws();
	const int L = lanes[0]->MOD_SYM_LEN;
	auto work = [&](int lo, int hi) {
		for (int i = lo; i < hi; i++) {
			CComm &c = *lanes[i];
			for (int f = 0; f < frames; f++) {
				const size_t b = (size_t)f * P + i;
				state[b * 3 + 0] = (unsigned int)(c.Rand.IX % 61967ul);
				state[b * 3 + 1] = (unsigned int)(c.Rand.IY % 63443ul);
				state[b * 3 + 2] = (unsigned int)(c.Rand.IZ % 63599ul);
				c.FrontEndToChannel();
				for (int s = 0; s < L; s++) {
					rx[(b * L + s) * 2] = c.RX_MOD_SYM[s].Real;
					rx[(b * L + s) * 2 + 1] = c.RX_MOD_SYM[s].Image;
					gain[(b * L + s) * 2] = c.GAIN[s].Real;
					gain[(b * L + s) * 2 + 1] = c.GAIN[s].Image;
					tx_index[b * L + s] = c.TX_MOD_IDX[s];
				}
			}
		}
	};
	int T = (int)std::thread::hardware_concurrency();
	if (const char *e = getenv("NBL_HOST_THREADS")) T = atoi(e);
	if (T > 16) T = 16;
	if (T > P) T = P;
	if (T <= 1) work(0, P);
	else {
		std::vector<std::thread> th;
		for (int t = 0; t < T; t++) th.emplace_back(work, (int)((long long)P * t / T), (int)((long long)P * (t + 1) / T));
		for (auto &x : th) x.join();
	}
	return L;
}

// The host layer's demodulators with gains on B frames (include/nbldpc.h, "demodulators with gains"): rx, gain [B][L][2] -> out
// [B][N][2^p - 1].  path 0: the general demodulator (src [N p] label-bit indices, prior [B][N p] or NULL, metric NBL_DEMOD_*);
// path 1: BPSK (src [N p] sample indices); path 2: one point per symbol (src [N] sample indices, M = 2^p).  gain == NULL: the
// gain-less functions (general path only).  No GPU, no profile.
int nblh_demod_csi(int path, int N, int p, int M, int L, const double *cons, const int *src, const double *rx, const double *gain,
                   const double *prior, double sigma, int metric, int B, double *out)
{
	if (N <= 0 || p < 1 || p > 8 || L <= 0 || B < 0 || path < 0 || path > 2) return -1;
	const size_t w = (size_t)(1 << p) - 1;
	if (path == 0) {
		if (M < 2 || M > 256 || (M & (M - 1)) || (metric != 0 && metric != 1)) return -1;
		int m = 0;
		while ((1 << m) < M) m++;
		std::vector<char> seen((size_t)L * m, 0);
		for (int i = 0; i < N * p; i++) {
			if (src[i] < 0) continue;
			if (src[i] >= L * m || seen[src[i]]) return -2;
			seen[src[i]] = 1;
		}
		for (int b = 0; b < B; b++)
			CComm::DemodulateGeneral(N, p, M, L, cons, src, rx + (size_t)b * L * 2, gain ? gain + (size_t)b * L * 2 : nullptr, sigma, metric,
			                         prior ? prior + (size_t)b * N * p : nullptr, out + (size_t)b * N * w);
		return 0;
	}
	if (!gain) return -1;
	const int nsrc = path == 1 ? N * p : N;
	for (int i = 0; i < nsrc; i++)
		if (src[i] >= L) return -2;
	if (path == 2 && M != (1 << p)) return -1;
	for (int b = 0; b < B; b++) {
		if (path == 1) CComm::DemodulateBpskCsi(N, p, src, rx + (size_t)b * L * 2, gain + (size_t)b * L * 2, sigma, out + (size_t)b * N * w);
		else CComm::DemodulateQaryCsi(N, 1 << p, cons, src, rx + (size_t)b * L * 2, gain + (size_t)b * L * 2, sigma, out + (size_t)b * N * w);
	}
	return 0;
}

// CComm::DemodulateGeneral on B frames: rx [B][L][2] -> out [B][N][2^p - 1].  No GPU, no profile.
int nblh_demod_general(int N, int p, int M, int L, const double *cons, const int *src, const double *rx, double sigma, int metric, int B, double *out)
{
	if (N <= 0 || p < 1 || p > 8 || M < 2 || M > 256 || (M & (M - 1)) || L <= 0 || (metric != 0 && metric != 1)) return -1;
	int m = 0;
	while ((1 << m) < M) m++;
	std::vector<char> seen((size_t)L * m, 0);
	for (int i = 0; i < N * p; i++) {
		if (src[i] < 0) continue;
		if (src[i] >= L * m || seen[src[i]]) return -2;
		seen[src[i]] = 1;
	}
	for (int b = 0; b < B; b++)
		CComm::DemodulateGeneral(N, p, M, L, cons, src, rx + (size_t)b * L * 2, sigma, metric, out + (size_t)b * N * ((1 << p) - 1));
	return 0;
}

// The prior-aware overload of CComm::DemodulateGeneral on B frames: prior [B][N p] (NULL: the function above).
int nblh_demod_general_prior(int N, int p, int M, int L, const double *cons, const int *src, const double *rx, const double *prior, double sigma,
                             int metric, int B, double *out)
{
	if (!prior) return nblh_demod_general(N, p, M, L, cons, src, rx, sigma, metric, B, out);
	if (N <= 0 || p < 1 || p > 8 || M < 2 || M > 256 || (M & (M - 1)) || L <= 0 || (metric != 0 && metric != 1)) return -1;
	int m = 0;
	while ((1 << m) < M) m++;
	std::vector<char> seen((size_t)L * m, 0);
	for (int i = 0; i < N * p; i++) {
		if (src[i] < 0) continue;
		if (src[i] >= L * m || seen[src[i]]) return -2;
		seen[src[i]] = 1;
	}
	for (int b = 0; b < B; b++)
		CComm::DemodulateGeneral(N, p, M, L, cons, src, rx + (size_t)b * L * 2, sigma, metric, prior + (size_t)b * N * p,
		                         out + (size_t)b * N * ((1 << p) - 1));
	return 0;
}

// Full simulation of one profile on the GPU; per Eb/N0 point: EbN0, errFrame, errSym, errBit, U_errFrame, frames, BER, SER, FER.
int nblh_simulate(const char *profile, int device, double *rows, int max_rows)
{
	CLink link;
	// device = -2: rehearsal of the multi-GPU split on a one-GPU box (two decoders, both on device 0)
	const std::vector<int> devs = device == -2 ? std::vector<int>{0, 0} : std::vector<int>{device};
	if (!link.Initial(profile, devs)) return -1;
	int n = 0;
	while (link.sim.NextSNR()) {
		if (!link.RunPoint(false)) return -2;
		if (n < max_rows) {
			double *r = rows + 9 * n;
			r[0] = link.sim.EbN0; r[1] = link.sim.errFrame; r[2] = link.sim.errSym; r[3] = link.sim.errBit; r[4] = link.sim.U_errFrame;
			r[5] = (link.sim.simCycle - 1) * link.sim.parallel; r[6] = link.sim.BER; r[7] = link.sim.SER; r[8] = link.sim.FER;
		}
		n++;
	}
	return n;
}

// the encoder of a profile's code as a dense map gen [N][K] (CNBLDPC::Generator); no GPU
int nblh_generator(const char *profile, unsigned short *gen_out)
{
	CSimulation sim;
	if (sim.Initial(profile) != 0) return -1;
	CNBLDPC code;
	if (!code.Initial(sim, -1)) return -2;
	std::vector<uint16_t> gen;
	if (!code.Generator(gen)) return -3;
	memcpy(gen_out, gen.data(), gen.size() * sizeof(uint16_t));
	return 0;
}

// TakeDecoded + ErrCount of the host chain (Comm.cpp:421-493) for `count` frames: tx_msg [count][K] the transmitted message symbols
// as Encode left them, decoded [count][N] -> err_sym, err_bit, crc_ok per frame.  No GPU.
int nblh_err_count(const char *profile, const int *tx_msg, const int *decoded, int count, int *err_sym, int *err_bit, int *crc_ok)
{
	CSimulation sim;
	if (sim.Initial(profile) != 0) return -1;
	CNBLDPC code;
	if (!code.Initial(sim, -1)) return -2;
	CComm c;
	if (!c.Initial(sim, 0, &code)) return -3;
	const int N = code.CodeLen, K = N - code.ChkLen, p = c.Bit_Len_PerSYM;
	for (int f = 0; f < count; f++) {
		for (int s = 0; s < K; s++) {
			c.TX_MSG_SYM[s] = tx_msg[(size_t)f * K + s];
			for (int k = 0; k < p; k++) c.TX_MSG_BIT[s * p + k] = (c.TX_MSG_SYM[s] >> k) & 1;
		}
		c.TakeDecoded(decoded + (size_t)f * N, true);
		double es = 0, eb = 0;
		int ok = 0;
		c.ErrCount(-1, es, eb, ok);
		err_sym[f] = (int)es; err_bit[f] = (int)eb; crc_ok[f] = ok;
	}
	return 0;
}

// CComm::CRCEncode on n bits (one int each): out [n + len]
int nblh_crc_encode(const int *in, int n, int len, int type24, int *out)
{
	CComm c;
	c.CRCEncode(out, in, n, len, type24);
	return 0;
}

// the PN register clocked literally: `clocks` calls of CComm::GenPN from `state` (bit i = regPN[i]); returns the register
int nblh_pn_clock(int state, unsigned long long clocks)
{
	CComm c;
	c.pn = state & 2047;
	for (unsigned long long i = 0; i < clocks; i++) c.GenPN();
	return c.pn;
}

// each lane's PN register in front of its first frame at an Eb/N0 point (ResetSources: the initial contents advanced `lane` clocks)
int nblh_pn_initial(int lane)
{
	CComm c;
	CSimulation sim;
	sim.parallel = 1;
	c.SetEbN0(sim, lane);
	return c.pn;
}

// encoder check: encode `count` random messages, return 0 if every codeword satisfies every parity check
int nblh_encode(const char *profile, const int *msg, int count, int *code_out)
{
	CSimulation sim;
	if (sim.Initial(profile) != 0) return -1;
	CNBLDPC code;
	if (!code.Initial(sim, -1)) return -2;
	const int N = code.CodeLen, K = N - code.ChkLen;
	std::vector<int> m(K);
	for (int c = 0; c < count; c++) {
		memcpy(m.data(), msg + (size_t)c * K, sizeof(int) * K);
		code.Encode(m.data(), code_out + (size_t)c * N);
	}
	return 0;
}
}
