// nbldpc_amd/host/comm.h -- CComm: one lane of the reference's link chain (Comm.h / Comm.cpp), minus the decoder it used to
// own: all lanes share one CNBLDPC (code parameters + encoder) and their frames are decoded together by the caller.
//   FrontEnd()    = GenerateMessage, Encode, Puncture, Modulate, Channel_AWGN, Demodulate      (Comm.cpp:181-189)
//                   (NBL_CHANNEL=rayleigh: Channel_Rayleigh in place of Channel_AWGN, and the demodulators take the lane's gains;
//                   include/nbldpc.h, "flat fading")
//   TakeDecoded() = the symbol/bit unpacking of CComm::Decode after NBLDPC.Decoding             (Comm.cpp:421-443)
//   Err()         = error counting                                                              (Comm.cpp:446-503)
#pragma once
#include <string>
#include <vector>
#include "nbldpc_host.h"
#include "rand.h"
#include "simulation.h"

struct CComplex { double Real = 0, Image = 0; };

class CComm {
public:
	int GFq = 0, parallel_num = 1, Bit_Len_PerSYM = 0;
	CNBLDPC *NBLDPC = nullptr;
	CRand Rand;
	int pn = 0;                        // the 11-stage PN register, bit i = regPN[i] of the reference (Comm.h)
	const unsigned short *pn_jump = nullptr; // state after `parallel - 1` clocks, per state (one look-up per message bit)
	int randomMsg = 0, crcLen = 0, crcLen_correct = 0;
	int MSG_SYM_LEN = 0, MSG_BIT_LEN = 0, CODE_SYM_LEN = 0, CODE_BIT_LEN = 0, PUN_SYM_LEN = 0, PUN_BIT_LEN = 0;
	int modOrder = 0, MOD_BIT_PER_SYM = 0, MOD_SYM_LEN = 0, MOD_BIT_LEN = 0;
	double CodeRate = 0, sigma_n = 0;
	int fade_model = 0, fade_block = 1; // NBL_FADING_* and the coherence in samples: NBL_CHANNEL=awgn|rayleigh (default awgn), NBL_FADE_BLOCK=k (default 1)
	std::vector<CComplex> GAIN;        // [MOD_SYM_LEN] the gain of every received sample of this frame (Channel_Rayleigh)
	int demod_metric = 0;              // NBL_DEMOD_* of the general demodulator (modOrder other than 2 and GFq): NBL_DEMOD_METRIC=maxlog|logsum
	std::vector<int> TX_MSG_BIT_beforeCRC, TX_MSG_BIT, TX_MSG_SYM, TX_CODE_SYM, TX_CODE_BIT, PUN_SYM, PUN_BIT, TX_MOD_BIT;
	std::vector<int> RX_DECODE_SYM, RX_DECODE_BIT, RX_MSG_SYM, RX_MSG_BIT;
	std::vector<CComplex> CONSTELLATION, TX_MOD_SYM, RX_MOD_SYM;
	std::vector<unsigned char> TX_MOD_IDX; // constellation index of every transmitted symbol (what Modulate looked up)
	std::vector<double> RX_LLR_BIT;
	std::vector<double> RX_LLR_SYM; // [CODE_SYM_LEN][GFq-1], row-major (the reference's double**)
	bool DecodeCorrect = false;

	bool Initial(CSimulation &sim, int parallel_order, CNBLDPC *shared);
	double SetEbN0(CSimulation &sim, int parallel_order);
	int FrontEnd();
	int FrontEndToChannel(); // everything up to Channel_AWGN: the demodulator runs on the device
	// everything up to Modulate: channel and demodulator run on the device.  The lane's generator state in front of the frame is
	// returned and the generator is moved past the uniform draws the channel would have made: ChannelDraws(), 4 * MOD_SYM_LEN for
	// Channel_AWGN (Comm.cpp:328-337).
	int FrontEndToModulate(unsigned int state_out[3]);
	// which received sample carries each code bit (BPSK) / code symbol (q-ary); any other order: which label bit t = s m + i carries
	// each code bit (kept bit k goes to t = k, -1 once k >= MOD_SYM_LEN m: the tail that MOD_SYM_LEN's floor drops)
	void DemodSource(std::vector<int> &src) const;
	bool GeneralDemod() const { return modOrder != 2 && modOrder != GFq; }
	// The general demodulator of include/nbldpc.h (nbl_set_demodulator_ex) restated literally, libm exp / log: N symbols of p bits, M
	// = 2^m points cons [M][2], src [N p], samples rx [L][2] -> out [N][2^p - 1].  src is taken as checked (each t once, below L m).
	static void DemodulateGeneral(int N, int p, int M, int L, const double *cons, const int *src, const double *rx, double sigma, int metric,
	                              double *out);
	// the prior-aware form (include/nbldpc.h, nbl_decode_batch_samples_prior): prior [N p] per code bit; NULL IS the function above
	static void DemodulateGeneral(int N, int p, int M, int L, const double *cons, const int *src, const double *rx, double sigma, int metric,
	                              const double *prior, double *out);
	// the gain-aware form (include/nbldpc.h, "demodulators with gains"): gain [L][2] per received sample, distances to the faded
	// points; prior as above (may be NULL); gain == NULL IS the function above
	static void DemodulateGeneral(int N, int p, int M, int L, const double *cons, const int *src, const double *rx, const double *gain, double sigma,
	                              int metric, const double *prior, double *out);
	// the BPSK and the one-point-per-symbol expressions with gains: src [N p] / [N] as DemodSource gives them, out [N][2^p - 1]
	static void DemodulateBpskCsi(int N, int p, const int *src, const double *rx, const double *gain, double sigma, double *out);
	static void DemodulateQaryCsi(int N, int q, const double *cons, const int *src, const double *rx, const double *gain, double sigma, double *out);
	int GenerateMessage();
	int GenPN();
	void CRCEncode(int *seqOut, const int *seqIn, int seqInLen, int crcLen, int crc24Type);
	int CrcCheck(const int *seqIn, int seqInLen, int crcLen, int crc24Type);
	int Encode();
	int Puncture();
	int Modulate();
	int Channel_AWGN();
	// Rayleigh block fading (include/nbldpc.h, nbl_set_fading): nblk = ceil(L / fade_block) gains first, two Rand_Norm(0, sqrt(0.5))
	// each, then the noise as Channel_AWGN draws it; RX = h * TX + n, the per-sample gains kept in GAIN
	int Channel_Rayleigh();
	int Channel() { return fade_model ? Channel_Rayleigh() : Channel_AWGN(); }
	unsigned long ChannelDraws() const // uniform draws one frame's channel makes: nbl_channel_draws
	{
		return 4ul * (unsigned long)MOD_SYM_LEN + (fade_model ? 4ul * (unsigned long)((MOD_SYM_LEN + fade_block - 1) / fade_block) : 0ul);
	}
	int Demodulate();
	int TakeDecoded(const int *decoded_sym, bool converged);
	int Err(CSimulation &sim);
	// Err() in two halves for the pipelined driver: HoldTx keeps the transmitted message of this cycle while the next cycle's
	// front-end already runs; ErrCount is lane-local (thread-safe); ErrAccumulate adds into the shared counters in lane order.
	void HoldTx(int slot);
	void ErrCount(int slot, double &errSym, double &errBit, int &crc_ok);
	static void ErrAccumulate(CSimulation &sim, double errSym, double errBit, int crc_ok);
	void ErrRates(CSimulation &sim) const;
	std::vector<int> HOLD_MSG_SYM[2], HOLD_MSG_BIT[2];
	std::string error;

private:
	void ResetSources(CSimulation &sim, int parallel_order);
	void SkipPN(int n); // clock the PN register n times (table walk)
	static const unsigned short *PnJumpTable(int n); // state -> state after n clocks (cached per n)
};
